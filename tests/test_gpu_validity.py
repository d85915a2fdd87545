"""Latent validity on the device (eae_amd.validity): `eae_class_dist_sums` through the C ABI by shape -- bit for bit against an int64
reference on integer data (tile edges, masking, segments and the self row, whatever the tolerance), within the derived bound of
tests/validity_ref.py on blobs -- its repeatability, then the Python layer against the NumPy references.

Bound (derived, not measured; validity_ref's module docstring): every (n, c) of every shape must lie within
sum_m pair(n, m) + (n_c + 2) 2^-24 sum_m d(n, m) of the float64 sum.  The silhouettes are held to the range that sums within that
bound can give (`silhouette_range`), plus the rounding of the float32 result.  Outputs and the workspace are poisoned before a call."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from kmeans_ref import U, blobs
from validity_ref import (SHAPES, calinski_harabasz_ref, case, case_ref, class_matrix_ref, clean_labels, davies_bouldin_ref, silhouette_range,
                          silhouette_ref, sums_by_label_ref)

pytestmark = pytest.mark.gpu

POISON = -7.0


def _dev(a, offset=False):
    """a on the device: a fresh allocation (16-byte aligned), or the same rows as a view that starts 4 bytes into one"""
    if not offset:
        return torch.from_numpy(np.array(a)).cuda()
    t = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")[1:].view(a.shape)
    t.copy_(torch.from_numpy(np.array(a)))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _c_sums(q, bank, seg, self_pos, metric, ws_bytes=None, ws_null=False, q_offset=False, bank_offset=False):
    """One call on a poisoned output and a workspace of NaN bit patterns: (rc, sums as NumPy)."""
    nq, width = q.shape
    m, k = bank.shape[0], len(seg) - 1
    lib = _lib.load()
    need = lib.eae_class_dist_workspace_bytes(nq, m, width, k)
    assert need >= 0
    qt, bt = _dev(q, q_offset), _dev(bank, bank_offset)
    st = torch.from_numpy(np.array(seg)).cuda()
    sp = None if self_pos is None else torch.from_numpy(np.array(self_pos)).cuda()
    sums = torch.full((nq, k), POISON, dtype=torch.float32, device="cuda")
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(nb, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.eae_class_dist_sums(_stream(), _ptr(qt), nq, _ptr(bt), m, width, _ptr(st), k, _ptr(sp), metric, _ptr(sums),
                                 None if ws_null else _ptr(ws), nb)
    return rc, sums.cpu().numpy()


def _sums(*args, **kw):
    rc, sums = _c_sums(*args, **kw)
    assert rc == 0, _lib.load().eae_last_error()
    return sums


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- 1. exact, by shape
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_integer_sums_are_exact(shape):
    """Squared distances of integer rows: every product, chain and running sum is an integer below 2^24, so fp32 is exact in any
    order and the sums must equal the int64 reference bit for bit -- NaN rows where the query is not finite and nowhere else, nothing
    leaking from the NaN rows that belong to no class."""
    q, bank, seg, self_pos = case(shape, "int")
    ref, _ = case_ref(shape, "int")
    whole = ref[~np.isnan(ref)]
    assert (whole < 2 ** 24).all() and np.array_equal(whole, np.round(whole))                  # the reference itself is integer and small
    assert np.isnan(bank[:seg[0]]).all() and np.isnan(bank[seg[-1]:]).all() and (shape[1] < 8 or seg[0] > 0 and seg[-1] < shape[1])
    got = _sums(q, bank, seg, self_pos, 1)
    assert np.array_equal(got.astype(np.float64), ref, equal_nan=True)
    assert np.array_equal(_bits(got), _bits(_sums(q, bank, seg, self_pos, 1)))                 # two runs, the same bits
    if shape[0] >= 3:
        assert np.isnan(got[1]).all() and not np.isnan(np.delete(got, 1, axis=0)).any()


@pytest.mark.parametrize("shape,cut", [((130, 600, 68, 3), True), ((40, 200, 8, 3), False)], ids=str)
def test_the_sums_do_not_depend_on_the_alignment_of_the_rows(shape, cut):
    """Rows of a width that is a multiple of 4 are staged with 16-byte loads from a 16-byte aligned base and float by float from any
    other, queries and bank each for itself: the four combinations give the same bits (staging changes no arithmetic), under both
    metrics and with a self row for every second query.  The first shape has two query tiles (the second of 2 rows), a class of
    nine tiles walked in three slices and two column passes (the second 4 wide); the second one pass, one slice and queries that
    are staged once per workgroup."""
    assert (_lib.load().eae_class_dist_workspace_bytes(*shape) > 0) == cut
    q, bank, seg, self_pos = case(shape, "int")
    ref, _ = case_ref(shape, "int")
    assert (ref[~np.isnan(ref)] < 2 ** 24).all()
    for metric in (1, 0):
        aligned = _sums(q, bank, seg, self_pos, metric)
        if metric == 1:
            assert np.array_equal(aligned.astype(np.float64), ref, equal_nan=True)     # exact, as test_integer_sums_are_exact
        for q_offset, bank_offset in ((False, True), (True, False), (True, True)):
            got = _sums(q, bank, seg, self_pos, metric, q_offset=q_offset, bank_offset=bank_offset)
            assert np.array_equal(_bits(got), _bits(aligned)), (metric, q_offset, bank_offset)


def test_the_shapes_cover_both_plans():
    need = [_lib.load().eae_class_dist_workspace_bytes(*shape) for shape in SHAPES]
    assert min(need) == 0 and max(need) > 0 and need[SHAPES.index((33, 70001, 64, 3))] > 0


# ---------------------------------------------------------------------------------------------------- 2. Euclidean, by shape
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_euclidean_sums_meet_the_bound(shape):
    q, bank, seg, self_pos = case(shape, "blobs")
    ref, bound = case_ref(shape, "blobs")
    got = _sums(q, bank, seg, self_pos, 0)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(got.astype(np.float64) - ref)
    print("worst share of the bound:", float((err[ok] / np.maximum(bound[ok], 1e-300)).max()))
    assert (err[ok] <= bound[ok]).all()                                    # every (n, c): none is left out
    assert (got[ok][ref[ok] == 0] == 0).all()                              # an empty class gives 0
    assert np.array_equal(_bits(got), _bits(_sums(q, bank, seg, self_pos, 0)))


def test_without_self_rows_and_with_rows_of_no_class_only():
    q, bank, seg, _ = case((129, 200, 20, 5), "int")
    ref = case_ref((129, 200, 20, 5), "int")[0]
    got = _sums(q, bank, seg, None, 1)                                     # self_pos = NULL: nothing is left out
    assert (got[0::2].astype(np.float64) == ref[0::2]).all() and (got[3::2].astype(np.float64) >= ref[3::2]).all()
    none = _sums(q, bank, np.full(6, 7, dtype=np.int64), None, 1)          # every class empty
    assert (np.delete(none, 1, axis=0) == 0).all() and np.isnan(none[1]).all()


def test_a_short_or_missing_workspace_is_rejected_and_nothing_is_written():
    q, bank, seg, self_pos = case((33, 70001, 64, 3), "int")
    lib = _lib.load()
    need = lib.eae_class_dist_workspace_bytes(33, 70001, 64, 3)
    assert need > 0
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_null=True)):
        rc, sums = _c_sums(q, bank, seg, self_pos, 1, **kw)
        assert rc == -2 and b"workspace" in lib.eae_last_error() and (sums == POISON).all()
    q, bank, seg, self_pos = case((129, 33, 3, 2), "int")                  # no workspace is needed where no segment is cut
    assert lib.eae_class_dist_workspace_bytes(129, 33, 3, 2) == 0
    rc, sums = _c_sums(q, bank, seg, self_pos, 1, ws_null=True)
    assert rc == 0 and np.array_equal(sums.astype(np.float64), case_ref((129, 33, 3, 2), "int")[0], equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 3. the Python layer
K = 6


@pytest.fixture(scope="module")
def labelled():
    """700 rows of width 24 in loose groups, labels unsorted in -1..5 with class 4 empty and class 5 a single row, one row of class 2
    holding an Inf and one label out of range.  Returns (z, labels) as NumPy and on the device."""
    rng = np.random.default_rng(31)
    labels = rng.integers(-1, 4, 700).astype(np.int64)
    z = (rng.standard_normal((700, 24)) + 0.8 * rng.standard_normal((5, 24))[labels + 1]).astype(np.float32) + np.float32(3.0)
    labels[10], labels[11] = 5, 17
    labels[20] = 2
    z[20, 3] = np.inf
    return z, labels, torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda()


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean"])
def test_class_distance_sums_against_the_reference(labelled, center, metric):
    z, labels, zt, lt = labelled
    q, qt = z[:150], zt[:150].clone()
    self_index = np.where(np.arange(150) % 3 == 0, np.arange(150), -1)
    sums, counts = eae_amd.class_distance_sums(qt, zt, lt, K, metric=metric, self_index=torch.from_numpy(self_index).cuda(), center=center)
    ref, rcounts, bound = sums_by_label_ref(q, z, labels, K, self_index, eae_amd.validity.METRICS.index(metric), center=center)
    assert sums.dtype == torch.float32 and counts.dtype == torch.int64 and counts.cpu().tolist() == rcounts.tolist() == [
        int((clean_labels(z, labels, K) == c).sum()) for c in range(K)]
    got = sums.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[20]).all() and np.isnan(got).sum() == K
    ok = ~np.isnan(ref)
    print("worst share of the bound:", float((np.abs(got - ref)[ok] / np.maximum(bound[ok], 1e-300)).max()))
    assert (np.abs(got - ref)[ok] <= bound[ok]).all()
    assert (np.delete(got[:, 4], 20) == 0).all()                           # the empty class
    again, _ = eae_amd.class_distance_sums(qt, zt, lt, K, metric=metric, self_index=torch.from_numpy(self_index).cuda(), center=center)
    assert torch.equal(again.view(torch.int32), sums.view(torch.int32))
    none, _ = eae_amd.class_distance_sums(qt, zt, lt, K, metric=metric, center=center)          # no self row
    nref, _, nbound = sums_by_label_ref(q, z, labels, K, None, eae_amd.validity.METRICS.index(metric), center=center)
    assert (np.abs(none.cpu().numpy() - nref)[ok] <= nbound[ok]).all()


def _silhouette_range(z, labels, rows, metric=0):
    """(ref, lo, hi) float64 [len(rows)]: the reference silhouettes of `rows` and the range the bound of the sums leaves around them;
    NaN for a row without a silhouette, 0 for a class of one row."""
    lab = clean_labels(z, labels, K)
    ref = silhouette_ref(z, labels, K, metric, rows)
    sums, counts, bound = sums_by_label_ref(z[rows], z, labels, K, rows, metric, center=True)
    own = lab[rows]
    live = (own >= 0) & (counts[np.maximum(own, 0)] > 1)
    lo, hi = ref.copy(), ref.copy()
    lo[live], hi[live] = silhouette_range(sums[live], counts, bound[live], own[live])
    assert (lo[live] <= ref[live]).all() and (ref[live] <= hi[live]).all() and (ref[(own >= 0) & ~live] == 0).all()
    return ref, lo, hi


def _silhouette_check(got, z, labels, rows, metric=0):
    """got float64 [len(rows)], row by row, with 4 * 2^-24 for the rounding of the float32 result (|s| <= 1)."""
    ref, lo, hi = _silhouette_range(z, labels, rows, metric)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert (got[ok] >= lo[ok] - 4 * U).all() and (got[ok] <= hi[ok] + 4 * U).all()
    return ref


def _matrix_check(got, z, labels, rows):
    """An entry is the fp32 mean over the n_a query rows of class a of sums / n_b: within the mean of those rows' bounds over n_b,
    and (n_a + 4) 2^-24 of the value for the division, the summation in some order, the mean's division and the diagonal's scale."""
    ref = class_matrix_ref(z, labels, K, rows)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    lab = clean_labels(z, labels, K)[rows]
    _, counts, bound = sums_by_label_ref(z[rows], z, labels, K, rows, 0, center=True)
    for a in range(K):
        for b in range(K):
            if not np.isnan(ref[a, b]):
                tol = bound[lab == a, b].mean() / (counts[b] - (a == b)) + ((lab == a).sum() + 4) * U * ref[a, b]
                assert abs(got[a, b] - ref[a, b]) <= tol, (a, b, got[a, b], ref[a, b], tol)
    return ref


def test_silhouette_samples_and_score(labelled):
    z, labels, zt, lt = labelled
    s = eae_amd.silhouette_samples(zt, lt, K)
    assert s.dtype == torch.float32 and s.shape == (700,)
    ref = _silhouette_check(s.cpu().numpy().astype(np.float64), z, labels, np.arange(700))
    assert np.isnan(ref[20]) and np.isnan(ref[11]) and ref[10] == 0 and np.isnan(ref[labels == -1]).all()
    auto = eae_amd.silhouette_samples(zt, torch.where(lt > 5, -1, lt))     # num_classes from labels.max(): 6 again
    assert torch.equal(auto.view(torch.int32), s.view(torch.int32))
    assert torch.equal(eae_amd.silhouette_samples(zt, lt, K).view(torch.int32), s.view(torch.int32))        # repeatable
    sq = eae_amd.silhouette_samples(zt, lt, K, metric="sqeuclidean")
    _silhouette_check(sq.cpu().numpy().astype(np.float64), z, labels, np.arange(700), metric=1)
    score, per_class = eae_amd.silhouette_score(zt, lt, K)
    assert score.dtype == torch.float64 and score.dim() == 0 and per_class.dtype == torch.float64 and per_class.shape == (K,)
    s64 = s.cpu().numpy().astype(np.float64)
    lab = clean_labels(z, labels, K)
    assert abs(float(score) - np.nanmean(s64)) <= 1e-6
    for c in range(K):
        if (lab == c).any():
            assert abs(float(per_class[c]) - s64[lab == c].mean()) <= 1e-6
        else:
            assert np.isnan(float(per_class[c]))
    # fewer than two non-empty classes: NaN everywhere, nothing raised
    assert torch.isnan(eae_amd.silhouette_samples(zt, torch.zeros_like(lt), 3)).all()
    assert torch.isnan(eae_amd.silhouette_score(zt, torch.zeros_like(lt), 3)[0])


def test_sample_takes_the_rows_of_the_stated_permutation(labelled):
    z, labels, zt, lt = labelled
    for seed, n in ((0, 64), (5, 699)):
        rows = torch.randperm(700, generator=torch.Generator().manual_seed(seed))[:n].numpy()
        _, lo, hi = _silhouette_range(z, labels, rows)
        score, per_class = eae_amd.silhouette_score(zt, lt, K, sample=n, seed=seed)
        assert np.nanmean(lo) - 4 * U <= float(score) <= np.nanmean(hi) + 4 * U
        lab = clean_labels(z, labels, K)[rows]
        for c in range(K):
            if (lab == c).any():
                assert lo[lab == c].mean() - 4 * U <= float(per_class[c]) <= hi[lab == c].mean() + 4 * U
            else:
                assert np.isnan(float(per_class[c]))
        if n == 64:                                                        # and they are not the rows of another seed
            other = torch.randperm(700, generator=torch.Generator().manual_seed(seed + 1))[:n].numpy()
            _, olo, ohi = _silhouette_range(z, labels, other)
            assert not np.nanmean(olo) - 4 * U <= float(score) <= np.nanmean(ohi) + 4 * U
    rows = torch.randperm(700, generator=torch.Generator().manual_seed(0))[:64].numpy()
    _matrix_check(eae_amd.class_distance_matrix(zt, lt, K, sample=64, seed=0).cpu().numpy().astype(np.float64), z, labels, rows)


def test_class_distance_matrix(labelled):
    z, labels, zt, lt = labelled
    m = eae_amd.class_distance_matrix(zt, lt, K)
    assert m.dtype == torch.float32 and m.shape == (K, K)
    assert torch.equal(eae_amd.class_distance_matrix(zt, lt, K).view(torch.int32), m.view(torch.int32))     # bitwise repeatable
    ref = _matrix_check(m.cpu().numpy().astype(np.float64), z, labels, np.arange(700))
    assert np.isnan(ref[4]).all() and np.isnan(ref[:, 4]).all() and np.isnan(ref[5, 5]) and not np.isnan(ref[:4, :4]).any()
    per_class = eae_amd.silhouette_score(zt, lt, K)[1]
    text = eae_amd.separation_table(m, per_class)
    assert len(text.splitlines()) == 2 + K and text.splitlines()[2 + 4].split() == ["4"] + ["-"] * 5


def test_the_two_indices(labelled):
    z, labels, zt, lt = labelled
    db, ch = eae_amd.davies_bouldin_score(zt, lt, K), eae_amd.calinski_harabasz_score(zt, lt, K)
    assert db.dtype == ch.dtype == torch.float64 and db.dim() == ch.dim() == 0
    rdb, rch = davies_bouldin_ref(z, labels, K), calinski_harabasz_ref(z, labels, K)
    assert abs(float(db) - rdb) <= 1e-9 * rdb and abs(float(ch) - rch) <= 1e-9 * rch
    assert float(eae_amd.davies_bouldin_score(zt, lt, K)) == float(db) and float(eae_amd.calinski_harabasz_score(zt, lt, K)) == float(ch)
    one = torch.zeros_like(lt)
    assert torch.isnan(eae_amd.davies_bouldin_score(zt, one, 3)) and torch.isnan(eae_amd.calinski_harabasz_score(zt, one, 3))


@pytest.mark.parametrize("criterion", ["silhouette", "calinski_harabasz", "davies_bouldin"])
def test_select_k_finds_the_six_blobs(criterion):
    """blobs(2000, 64, 6, 0): test_validity_reference shows in float64 that 6 wins under each criterion by more than the bound."""
    z = torch.from_numpy(blobs(2000, 64, 6, 0)[0]).cuda()
    best, scores, results = eae_amd.select_k(z, (2, 4, 6, 8, 10), criterion=criterion)
    assert best == 6 and sorted(scores) == sorted(results) == [2, 4, 6, 8, 10], scores
    assert results[6].centroids.shape == (6, 64) and all(isinstance(v, float) for v in scores.values())
    if criterion == "silhouette":
        sampled = eae_amd.select_k(z, (4, 6, 8), sample=500, seed=3)
        assert sampled[0] == 6 and abs(sampled[1][6] - scores[6]) < 0.01
