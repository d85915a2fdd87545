"""NumPy float64 restatement of the latent-validity functions (include/eae.h, "latent validity"; eae_amd.validity) and the bound the
GPU tests compare `eae_class_dist_sums` with.  Nothing here is measured on the code under test.

The bound (derived from the fp32 format; `sums_ref` returns it per (n, c)).  The kernel computes a pair's squared distance as
max(0, fma(-2, q.b, ||b||^2) + ||q||^2) in fp32.  tau_n = kmeans_ref.tau(q, bank)[n] = 4 (L + 2) 2^-24 (||q_n|| + max_m ||b_m||)^2 is
the bound of a COMPARISON of two such scores (DESIGN.md sections 21 and 23), so each fp32 d^2 is within
    e2 = tau_n / 2
of the float64 value (the clamp at 0 moves it towards the truth, which is >= 0).  With d the float64 distance, the square root of a
number within e2 of d^2 lies within max(sqrt(d^2 + e2) - d, d - sqrt(max(0, d^2 - e2))) of d, and a correctly rounded `sqrtf` adds at
most 2^-24 d (the figure is taken at the float64 d: the difference is of second order in 2^-24):
    pair(n, m) = max(sqrt(d^2 + e2) - d, d - sqrt(max(0, d^2 - e2))) + 2^-24 d.
Under the squared metric there is no root: pair(n, m) = e2.  A sum of n_c such terms in fp32, in any order, adds at most
(n_c - 1) 2^-24 of the sum of the terms' magnitudes; (n_c + 2) 2^-24 sum d leaves room for the masked zeros, the add of the two lanes
of a query and the adds of the slices' partial sums:
    bound(n, c) = sum_m pair(n, m) + (n_c + 2) 2^-24 sum_m d(n, m).
The bound is loose near d = 0 (there sqrt(e2) dominates) and tight elsewhere; the exact integer tests carry the structural weight.

`center=True` of `class_distance_sums` subtracts one fp32 vector mu from both sides.  Distances do not depend on mu, and
fl(x - mu) = (x - mu)(1 + delta), |delta| <= 2^-24 per coordinate, moves a row by at most 2^-24 ||x - mu||: the kernel's inputs are
then within that of the exact centred rows, a pair's distance within 2^-24 (||q_n - mu|| + ||b_m - mu||).  `sums_by_label_ref` takes
tau of the centred rows and adds that term per pair.
"""
import functools

import numpy as np

from kmeans_ref import U, blobs, finite_rows, tau

# (Nq, M, L, K): the query-tile boundary, most classes empty or singletons, wide rows, the slice path of long segments
SHAPES = [(1, 1, 1, 1), (129, 33, 3, 2), (127, 200, 20, 5), (128, 200, 20, 5), (129, 200, 20, 5), (257, 300, 128, 256), (300, 1031, 256, 7),
          (1000, 4096, 64, 10), (33, 70001, 64, 3)]
BANK_TILE = 64


def _d2(q, b, chunk=1 << 22):
    """float64 [Nq, M] squared distances by differences (no cancellation: equal rows give exactly 0), a block of queries at a time."""
    q = np.asarray(q, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    out = np.empty((q.shape[0], b.shape[0]))
    step = max(1, chunk // max(1, b.shape[0] * b.shape[1]))
    for lo in range(0, q.shape[0], step):
        diff = q[lo:lo + step, None, :] - b[None, :, :]
        out[lo:lo + step] = np.einsum("nml,nml->nm", diff, diff)
    return out


def pair_bound(d2, e2, metric):
    """The bound of one pair's fp32 distance (module docstring): d2 float64 [Nq, M], e2 [Nq, 1]."""
    if metric == 1:
        return np.broadcast_to(e2, d2.shape)
    d = np.sqrt(d2)
    return np.maximum(np.sqrt(d2 + e2) - d, d - np.sqrt(np.maximum(d2 - e2, 0.0))) + U * d


def sums_ref(q, bank, seg, self_pos=None, metric=0, extra=None, seen=None):
    """(sums float64 [Nq, K], bound [Nq, K]) of `eae_class_dist_sums` on a bank sorted by class: rows seg[c] .. seg[c+1]-1 are class
    c, rows outside [seg[0], seg[K]) are never looked at; self_pos[n] (or -1) is left out of row n; metric 0 Euclidean, 1 squared.  A
    query row with a NaN or an Inf gets NaN (sums and bound); an empty class gives 0 with bound 0.
    extra: float64 [Nq, M] or None, added to every pair's bound (the centring term of `sums_by_label_ref`); seen: (q', bank') or None,
    translates of q and bank that the kernel is given instead: tau is taken from their norms (the distances are the same)."""
    q = np.asarray(q, dtype=np.float64)
    bank = np.asarray(bank, dtype=np.float64)
    seg = np.asarray(seg, dtype=np.int64)
    k = seg.shape[0] - 1
    nq = q.shape[0]
    ok = finite_rows(q)
    sums = np.zeros((nq, k))
    bound = np.zeros((nq, k))
    lo, hi = int(seg[0]), int(seg[k])
    if hi > lo:
        assert finite_rows(bank[lo:hi]).all(), "bank rows inside a segment must be finite"
        e2 = np.zeros((nq, 1))
        tq, tb = (q, bank) if seen is None else (np.asarray(seen[0], dtype=np.float64), np.asarray(seen[1], dtype=np.float64))
        e2[ok, 0] = tau(tq[ok], tb[lo:hi]) / 2.0
    for c in range(k):
        a, b = int(seg[c]), int(seg[c + 1])
        if b <= a:
            continue
        d2 = np.zeros((nq, b - a))
        d2[ok] = _d2(q[ok], bank[a:b])
        d = d2 if metric == 1 else np.sqrt(d2)
        pb = pair_bound(d2, e2, metric).copy()
        if extra is not None:
            pb += extra[:, a:b]
        if self_pos is not None:
            sp = np.asarray(self_pos, dtype=np.int64)
            hit = np.nonzero((sp >= a) & (sp < b))[0]
            d = d.copy()
            d[hit, sp[hit] - a] = 0.0
            pb[hit, sp[hit] - a] = 0.0
        sums[:, c] = d.sum(1)
        bound[:, c] = pb.sum(1) + (b - a + 2) * U * d.sum(1)
    sums[~ok] = np.nan
    bound[~ok] = np.nan
    return sums, bound


def clean_labels(rows, labels, k):
    """Labels with -1 for every row that joins no class: labelled outside [0, k), or not finite."""
    labels = np.asarray(labels, dtype=np.int64)
    return np.where(finite_rows(rows) & (labels >= 0) & (labels < k), labels, -1)


def sums_by_label_ref(q, bank, labels, k, self_index=None, metric=0, center=True):
    """`validity.class_distance_sums` in float64: (sums [Nq, K], counts [K], bound [Nq, K]).  The distances are those of the rows as
    given; the bound is taken on the rows the kernel sees (centred or not) and, when centred, carries the centring term."""
    q64 = np.asarray(q, dtype=np.float64)
    b64 = np.asarray(bank, dtype=np.float64)
    lab = clean_labels(b64, labels, k)
    order = np.argsort(lab, kind="stable")
    counts = np.bincount(lab[lab >= 0], minlength=k).astype(np.int64)
    seg = np.concatenate([[len(lab) - counts.sum()], counts]).cumsum()
    inv = np.empty(len(lab), dtype=np.int64)
    inv[order] = np.arange(len(lab))
    self_pos = None
    if self_index is not None:
        si = np.asarray(self_index, dtype=np.int64)
        self_pos = np.where(si >= 0, inv[np.clip(si, 0, len(lab) - 1)], -1)
    extra, seen = None, None
    if center and counts.sum() > 0:
        mu = b64[lab >= 0].mean(0)
        okq = finite_rows(q64)
        qk = np.where(okq[:, None], q64 - mu, np.nan)
        bk = np.where((lab >= 0)[:, None], b64 - mu, np.nan)
        qn = np.where(okq, np.sqrt(np.nansum(qk ** 2, 1)), 0.0)
        bn = np.where(lab >= 0, np.sqrt(np.nansum(bk ** 2, 1)), 0.0)
        extra = U * (qn[:, None] + bn[order][None, :])
        if metric == 1:                                         # d^2 moves by at most 2 d delta + delta^2, d <= ||q|| + ||b||
            extra = extra * (2.0 * (qn[:, None] + bn[order][None, :]) + extra)
        seen = (qk, bk[order])
    sums, bound = sums_ref(q64, b64[order], seg, self_pos, metric, extra, seen)
    return sums, counts, bound


def silhouette_ref(z, labels, k, metric=0, rows=None):
    """float64 [N] (or [len(rows)]): the silhouette of every row (of the rows `rows`) against all of z, with `silhouette_samples`'
    conventions: a class of one row 0, max(a, b) = 0 gives 0, a row of no class NaN, fewer than two non-empty classes NaN everywhere."""
    z = np.asarray(z, dtype=np.float64)
    lab = clean_labels(z, labels, k)
    rows = np.arange(z.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    sums, counts, _ = sums_by_label_ref(z[rows], z, lab, k, rows, metric, center=False)
    out = np.full(len(rows), np.nan)
    if (counts > 0).sum() < 2:
        return out
    for j, n in enumerate(rows):
        c = lab[n]
        if c < 0:
            continue
        if counts[c] == 1:
            out[j] = 0.0
            continue
        a = sums[j, c] / (counts[c] - 1)
        b = min(sums[j, o] / counts[o] for o in range(k) if o != c and counts[o] > 0)
        out[j] = 0.0 if max(a, b) == 0 else (b - a) / max(a, b)
    return out


def silhouette_range(sums, counts, bound, own):
    """(lo, hi) float64 [Nq]: the least and greatest silhouette that sums within `bound` of `sums` can give for rows of class own[n]
    (>= 0, of more than one row, two non-empty classes): s falls with a and rises with b, and b rises with every other class's sum."""
    k = sums.shape[1]
    mine = np.arange(k)[None, :] == own[:, None]
    out = []
    for sign in (+1.0, -1.0):
        moved = np.maximum(sums + sign * bound * np.where(mine, 1.0, -1.0), 0.0)
        a = moved[np.arange(len(own)), own] / (counts[own] - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            b = np.where(mine | (counts[None, :] == 0), np.inf, moved / counts[None, :]).min(1)
            out.append(np.where(np.maximum(a, b) > 0, (b - a) / np.maximum(a, b), 0.0))
    return out[0], out[1]


def class_matrix_ref(z, labels, k, rows=None):
    """float64 [K, K]: mean Euclidean distance from the rows of class a (among `rows`) to the rows of class b, the diagonal over
    distinct pairs; NaN for an empty class, a class without a query row, and the diagonal of a class of one row."""
    z = np.asarray(z, dtype=np.float64)
    lab = clean_labels(z, labels, k)
    rows = np.arange(z.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    sums, counts, _ = sums_by_label_ref(z[rows], z, lab, k, rows, 0, center=False)
    out = np.full((k, k), np.nan)
    for a in range(k):
        mine = lab[rows] == a
        if not mine.any():
            continue
        for b in range(k):
            n = counts[b] - (a == b)
            if counts[b] > 0 and n > 0:
                out[a, b] = sums[mine, b].mean() / n
    return out


def _class_means(z, lab, k):
    return [z[lab == c].mean(0) for c in range(k) if (lab == c).any()], [z[lab == c] for c in range(k) if (lab == c).any()]


def davies_bouldin_ref(z, labels, k):
    z = np.asarray(z, dtype=np.float64)
    cent, rows = _class_means(z, clean_labels(z, labels, k), k)
    if len(cent) < 2:
        return np.nan
    s = [np.sqrt(((r - c) ** 2).sum(1)).mean() for c, r in zip(cent, rows)]
    worst = []
    for i in range(len(cent)):
        r = [(s[i] + s[j]) / np.sqrt(((cent[i] - cent[j]) ** 2).sum()) for j in range(len(cent))
             if j != i and ((cent[i] - cent[j]) ** 2).sum() > 0]
        worst.append(max(r) if r else 0.0)
    return float(np.mean(worst))


def calinski_harabasz_ref(z, labels, k):
    z = np.asarray(z, dtype=np.float64)
    lab = clean_labels(z, labels, k)
    cent, rows = _class_means(z, lab, k)
    if len(cent) < 2:
        return np.nan
    n = int((lab >= 0).sum())
    mean = z[lab >= 0].mean(0)
    between = sum(len(r) * ((c - mean) ** 2).sum() for c, r in zip(cent, rows))
    within = sum(((r - c) ** 2).sum() for c, r in zip(cent, rows))
    return 1.0 if within == 0 else float(between * (n - len(cent)) / (within * (len(cent) - 1)))


# ---------------------------------------------------------------------------------------------------- the cases of the kernel tests
def segments(m, k):
    """seg int64 [K+1] of a bank of m rows, as far as the shape admits: one unclassed row before the first and at least one after
    the last segment; class 0 ends one row past a 64-row tile (length = 1 mod 64); class 1 is empty between two non-empty ones; class
    2 (the last class when K = 2) ends one row short of a tile (length 63); the other classes share the rest -- with K = 256 and 300
    rows they are singletons and empties -- and with K <= 3 the rest lengthens class 0 by whole tiles: the long segment."""
    pad = 1 if m >= 8 else 0
    a = m - 2 * pad
    lens = [0] * k
    if k == 1:
        lens[0] = a
    elif a < 128:
        lens[0], lens[-1] = 1, a - 1
    else:
        lens[0], lens[min(2, k - 1)] = 65, 63
        rest, others = a - 128, list(range(3, k))
        if others:
            for j, c in enumerate(others):
                lens[c] = rest // len(others) + (j < rest % len(others))
        else:
            lens[0] += rest // BANK_TILE * BANK_TILE
    return pad + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(q, bank, seg, self_pos) of one shape, all NumPy, computed once: kind "int" -- coordinates in -4..4, thinned for long segments
    so that every sum of squared distances stays below 2^24 -- or "blobs" (kmeans_ref.blobs, norm about 4) with one query equal to a
    bank row of class 0.  The unclassed bank rows are NaN, every second query has a self_pos inside [seg[0], seg[K]), and (from 3
    queries on) query 1 holds an Inf."""
    nq, m, width, k = shape
    rng = np.random.default_rng(nq + 3 * m + 5 * width + 7 * k)
    seg = segments(m, k)
    if kind == "int":
        longest = int(np.diff(seg).max())
        keep = min(1.0, 2.0 ** 23 / (longest * width * 13.4))              # E d^2 = 2 L p 60 / 9 per pair
        rows = (rng.integers(-4, 5, (nq + m, width)) * (rng.random((nq + m, width)) < keep)).astype(np.float32)
    else:
        rows = blobs(nq + m, width, min(k, 6), nq + m)[0]
    q, bank = rows[:nq].copy(), rows[nq:].copy()
    if kind == "blobs" and seg[1] > seg[0]:
        q[0] = bank[seg[0]]                                                # a pair at distance 0, where the bound is loosest
    bank[:seg[0]] = np.nan
    bank[seg[k]:] = np.nan
    self_pos = np.full(nq, -1, dtype=np.int64)
    self_pos[1::2] = seg[0] + (np.arange(nq)[1::2] * 7) % max(int(seg[k] - seg[0]), 1)
    if nq >= 3:
        q[1, width // 2] = np.inf
    q.setflags(write=False), bank.setflags(write=False), seg.setflags(write=False), self_pos.setflags(write=False)
    return q, bank, seg, self_pos


@functools.lru_cache(maxsize=None)
def case_ref(shape, kind):
    """(sums, bound) of `case(shape, kind)`: squared distances for "int", Euclidean for "blobs"."""
    q, bank, seg, self_pos = case(shape, kind)
    return sums_ref(q, bank, seg, self_pos, 1 if kind == "int" else 0)


def emulate_fp32(q, bank, seg, self_pos, metric):
    """The kernel's arithmetic in fp32 NumPy: an fp32 product for the dot products and fp32 sums for the norms (some order), fma's
    two roundings in place of one, `max`, `sqrt`, and an fp32 running sum per (n, c)."""
    k = len(seg) - 1
    out = np.zeros((q.shape[0], k), dtype=np.float32)
    ok = finite_rows(q)
    qn = (q * q).sum(1, dtype=np.float32)
    for c in range(k):
        a, b = int(seg[c]), int(seg[c + 1])
        if b <= a:
            continue
        rows = bank[a:b]
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.maximum(np.float32(-2) * (q @ rows.T) + (rows * rows).sum(1, dtype=np.float32)[None, :] + qn[:, None], np.float32(0))
        d = d if metric == 1 else np.sqrt(d)
        hit = np.nonzero((self_pos >= a) & (self_pos < b))[0]
        d[hit, self_pos[hit] - a] = 0
        out[:, c] = d.sum(1, dtype=np.float32)
    out[~ok] = np.nan
    return out
