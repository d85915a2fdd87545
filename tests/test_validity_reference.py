"""Latent validity without a device: the NumPy references (tests/validity_ref.py) against scikit-learn and by hand, the acceptance
bound on an fp32 emulation of the kernel's arithmetic, the host-only half of the C ABI, and everything eae_amd.validity and
`report.separation_table` reject or compute on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from kmeans_ref import blobs, fit_ref
from validity_ref import (SHAPES, calinski_harabasz_ref, case, case_ref, class_matrix_ref, davies_bouldin_ref, emulate_fp32, segments,
                          silhouette_range, silhouette_ref, sums_by_label_ref, sums_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the references
def _labelled_blobs():
    """blobs(301, 64, 5, 0) under 7 class ids: class 3 reduced to a single row (the others of blob 3 join class 0), classes 5 empty."""
    z, ids, _ = blobs(301, 64, 5, 0)
    labels = ids.astype(np.int64).copy()
    labels[labels == 4] = 6
    three = np.nonzero(labels == 3)[0]
    labels[three[1:]] = 0
    return z, labels, 7


def test_silhouette_ref_agrees_with_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    z, labels, k = _labelled_blobs()
    assert (labels == 3).sum() == 1 and (labels == 5).sum() == 0 and (labels == 4).sum() == 0
    ours = silhouette_ref(z, labels, k)
    theirs = metrics.silhouette_samples(z.astype(np.float64), labels)
    assert np.abs(ours - theirs).max() <= 1e-9
    assert ours[labels == 3].tolist() == [0.0]
    sq = silhouette_ref(z, labels, k, metric=1)
    assert np.abs(sq - metrics.silhouette_samples(z.astype(np.float64), labels, metric="sqeuclidean")).max() <= 1e-9


def test_index_refs_agree_with_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    z, labels, k = _labelled_blobs()
    z64 = z.astype(np.float64)
    db, ch = davies_bouldin_ref(z, labels, k), calinski_harabasz_ref(z, labels, k)
    assert abs(db - metrics.davies_bouldin_score(z64, labels)) <= 1e-9 * max(1.0, abs(db))
    assert abs(ch - metrics.calinski_harabasz_score(z64, labels)) <= 1e-9 * max(1.0, abs(ch))


def test_refs_by_hand():
    z = np.array([[0.0], [1.0], [5.0], [np.nan], [9.0]])
    labels = np.array([0, 0, 1, 1, -1])
    sums, counts, _ = sums_by_label_ref(z, z, labels, 3, np.arange(5), center=False)
    assert counts.tolist() == [2, 1, 0]
    assert sums[:3].tolist() == [[1.0, 5.0, 0.0], [1.0, 4.0, 0.0], [9.0, 0.0, 0.0]] and np.isnan(sums[3]).all()
    assert sums[4].tolist() == [17.0, 4.0, 0.0]                            # an unclassed query still has sums
    s = silhouette_ref(z, labels, 3)
    assert s[:3].tolist() == [0.8, 0.75, 0.0] and np.isnan(s[3:]).all()
    assert np.isnan(silhouette_ref(z, np.array([0, 0, 0, 0, -1]), 3)).all()     # one non-empty class
    assert silhouette_ref(np.zeros((4, 2)), np.array([0, 0, 1, 1]), 2).tolist() == [0.0] * 4        # max(a, b) = 0
    m = class_matrix_ref(z, labels, 3)
    assert m[0, 0] == 1.0 and m[0, 1] == 4.5 and m[1, 0] == 4.5 and np.isnan(m[1, 1]) and np.isnan(m[2]).all() and np.isnan(m[:, 2]).all()
    # the segment form: rows outside [seg[0], seg[K]) are never looked at, the self row is left out
    bank = np.array([[np.nan], [0.0], [2.0], [7.0], [np.inf]])
    sums, bound = sums_ref(np.array([[1.0], [np.inf]]), bank, [1, 3, 3, 4], np.array([2, -1]), metric=1)
    assert sums[0].tolist() == [1.0, 0.0, 36.0] and np.isnan(sums[1]).all() and (bound[0] > 0).tolist() == [True, False, True]


def test_segments_carry_the_edges():
    for nq, m, width, k in SHAPES:
        seg = segments(m, k)
        lens = np.diff(seg)
        assert len(seg) == k + 1 and (lens >= 0).all() and seg[0] >= 0 and seg[k] <= m
        if m >= 200:
            assert seg[0] > 0 and seg[k] < m and lens[0] % 64 == 1 and 63 in lens.tolist()
        if m >= 200 and k >= 3:
            assert lens[1] == 0 and lens[0] > 0 and lens[2] > 0
    assert np.diff(segments(70001, 3)).max() > 64 * 1000                   # the long segment
    assert (np.diff(segments(300, 256)) <= 1).sum() >= 250                 # empties and singletons


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fp32_emulation_meets_the_bound(shape):
    """Required by the bound's derivation: fp32 arithmetic in another order than the kernel's stays within it for every (n, c), and on
    the integer data it is exact (every sum of squared distances below 2^24, as the GPU's exact test needs)."""
    q, bank, seg, self_pos = case(shape, "int")
    ref, _ = case_ref(shape, "int")
    assert np.nanmax(ref, initial=0.0) < 2 ** 24 and np.array_equal(ref[~np.isnan(ref)], np.round(ref[~np.isnan(ref)]))
    assert np.array_equal(emulate_fp32(q, bank, seg, self_pos, 1).astype(np.float64), ref, equal_nan=True)
    q, bank, seg, self_pos = case(shape, "blobs")
    ref, bound = case_ref(shape, "blobs")
    got = emulate_fp32(q, bank, seg, self_pos, 0).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isnan(ref), np.isnan(bound))
    ok = ~np.isnan(ref)
    assert (np.abs(got - ref)[ok] <= bound[ok]).all(), float((np.abs(got - ref)[ok] / np.maximum(bound[ok], 1e-300)).max())
    assert (bound[ok][ref[ok] > 0] > 0).all() and (bound[ok] >= 0).all()
    if shape[0] >= 3:
        assert np.isnan(ref[1]).all() and not np.isnan(ref[0]).any()


def test_the_bound_rejects_a_wrong_sum():
    q, bank, seg, self_pos = case((129, 200, 20, 5), "blobs")
    ref, bound = case_ref((129, 200, 20, 5), "blobs")
    far = int(seg[0] + np.argmax(((bank[seg[0]:seg[1]] - q[4]) ** 2).sum(1)))           # a row of class 0 in another blob than query 4
    short = bank.copy()
    short[far] = q[4]                                                      # distance 0 in place of the row's: as if it were left out
    assert abs(emulate_fp32(q, short, seg, self_pos, 0)[4, 0] - ref[4, 0]) > bound[4, 0]
    on = emulate_fp32(q, bank, seg, np.full_like(self_pos, -1), 0)         # the self row not excluded
    assert (np.abs(on - ref)[3::2] > bound[3::2]).any()


# ---------------------------------------------------------------------------------------------------- C ABI, host only
def test_new_symbols_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eae.h")).read(), flags=re.S)
    ctype = {"void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "const long long*": C.c_void_p, "long long": C.c_longlong,
             "int": C.c_int}
    for name in ("eae_class_dist_workspace_bytes", "eae_class_dist_sums"):
        ret, args = re.search(r"([a-z ]+?)\s+" + name + r"\s*\(([^)]*)\)\s*;", src).groups()
        types = [a.strip().rsplit(" ", 1)[0].strip() + ("*" if a.strip().rsplit(" ", 1)[1].startswith("*") else "") for a in args.split(",")]
        types = [t.replace(" *", "*") for t in types]
        assert name in _lib.EXPORTS and _lib._PROTOS[name] == (ctype[ret.strip()], [ctype[t] for t in types]), (name, ret, types)
    assert "latent validity" in open(os.path.join(ROOT, "include", "eae.h")).read()


def test_workspace_plan_is_host_only_and_deterministic():
    lib = _lib.load()
    sliced = {}
    for nq, m, width, k in SHAPES + [(1 << 17, 1 << 17, 64, 10), (1 << 17, 1 << 17, 64, 256), (8192, 1 << 20, 64, 10),
                                     (2 ** 31 - 1, 2 ** 31 - 1, 256, 256)]:
        b = lib.eae_class_dist_workspace_bytes(nq, m, width, k)
        assert b >= 0 and b % (4 * nq * k) == 0 and b // (4 * nq * k) <= 64, (nq, m, width, k, b)
        assert b == lib.eae_class_dist_workspace_bytes(nq, m, width, k) and b <= 128 << 20
        assert b == lib.eae_class_dist_workspace_bytes(nq, m, 1, k)        # a function of (Nq, M, K)
        sliced[nq, m, width, k] = b // (4 * nq * k)
    assert sliced[1, 1, 1, 1] == 0 and sliced[33, 70001, 64, 3] > 1 and sliced[1000, 4096, 64, 10] > 1      # both plans among the shapes
    assert sliced[1 << 17, 1 << 17, 64, 10] == 0 and sliced[8192, 1 << 20, 64, 10] > 1
    for nq, m, width, k in ((0, 5, 4, 1), (-1, 5, 4, 1), (2 ** 31, 5, 4, 1), (5, 0, 4, 1), (5, 2 ** 31, 4, 1), (5, 5, 0, 1), (5, 5, 257, 1),
                            (5, 5, 4, 0), (5, 5, 4, 257)):
        assert lib.eae_class_dist_workspace_bytes(nq, m, width, k) < 0 and b"class_dist" in lib.eae_last_error()


def test_sums_rejects_bad_arguments_before_any_launch():
    """EAE_ERR_ARG comes from the host-side checks: no device is touched (this test runs without one)."""
    lib = _lib.load()
    p = 0x1000          # never dereferenced on the host
    ws = 1 << 40
    for nq, m, width, k in ((0, 5, 4, 1), (2 ** 31, 5, 4, 1), (5, 0, 4, 1), (5, 2 ** 31, 4, 1), (5, 5, 0, 1), (5, 5, 257, 1), (5, 5, 4, 0),
                            (5, 5, 4, 257)):
        assert lib.eae_class_dist_sums(None, p, nq, p, m, width, p, k, p, 0, p, p, ws) == -2
    assert lib.eae_class_dist_sums(None, None, 5, p, 5, 4, p, 1, p, 0, p, p, ws) == -2
    assert lib.eae_class_dist_sums(None, p, 5, None, 5, 4, p, 1, p, 0, p, p, ws) == -2
    assert lib.eae_class_dist_sums(None, p, 5, p, 5, 4, None, 1, p, 0, p, p, ws) == -2
    assert lib.eae_class_dist_sums(None, p, 5, p, 5, 4, p, 1, p, 0, None, p, ws) == -2 and b"NULL" in lib.eae_last_error()
    for metric in (-1, 2):
        assert lib.eae_class_dist_sums(None, p, 5, p, 5, 4, p, 1, None, metric, p, p, ws) == -2 and b"metric" in lib.eae_last_error()
    need = lib.eae_class_dist_workspace_bytes(33, 70001, 64, 3)
    assert need > 0
    assert lib.eae_class_dist_sums(None, p, 33, p, 70001, 64, p, 3, None, 0, p, None, need) == -2
    assert lib.eae_class_dist_sums(None, p, 33, p, 70001, 64, p, 3, None, 0, p, p, need - 1) == -2 and b"workspace" in lib.eae_last_error()


# ---------------------------------------------------------------------------------------------------- Python rejections
def _z(n=20, width=8):
    return torch.zeros((n, width), dtype=torch.float32)


def _l(n=20):
    return torch.zeros(n, dtype=torch.int64)


def test_exports():
    for name in ("class_distance_sums", "silhouette_samples", "silhouette_score", "class_distance_matrix", "davies_bouldin_score",
                 "calinski_harabasz_score", "select_k"):
        assert name in eae_amd.__all__ and getattr(eae_amd, name) is getattr(eae_amd.validity, name)
    assert "separation_table" in eae_amd.__all__ and eae_amd.separation_table is eae_amd.report.separation_table


def _rejected(fn, kw, names):
    with pytest.raises(RuntimeError) as e:
        fn(**kw)
    assert "HIP device" not in str(e.value) and any(n in str(e.value) for n in names), str(e.value)


@pytest.mark.parametrize("kwargs,names", [
    (dict(q=torch.zeros((20, 8), dtype=torch.float64)), ["q "]), (dict(q=torch.zeros(8)), ["q "]), (dict(q=torch.zeros((20, 7))), ["width"]),
    (dict(q=np.zeros((20, 8), dtype=np.float32)), ["q "]), (dict(bank=torch.zeros((30, 8), dtype=torch.float16)), ["bank"]),
    (dict(bank=torch.zeros((0, 8))), ["bank"]), (dict(q=torch.zeros((4, 257)), bank=torch.zeros((30, 257))), ["width"]),
    (dict(q=torch.zeros((20, 8), device="meta")), ["bank on"]),
    (dict(labels=torch.zeros(29, dtype=torch.int64)), ["labels"]), (dict(labels=torch.zeros(30, dtype=torch.int32)), ["labels"]),
    (dict(labels=torch.zeros((30, 1), dtype=torch.int64)), ["labels"]), (dict(labels=[0] * 30), ["labels"]),
    (dict(labels=torch.zeros(30, dtype=torch.int64, device="meta")), ["labels"]),
    (dict(num_classes=0), ["num_classes"]), (dict(num_classes=257), ["num_classes"]), (dict(num_classes=2.0), ["num_classes"]),
    (dict(num_classes=True), ["num_classes"]), (dict(metric="cosine"), ["metric"]), (dict(metric=0), ["metric"]),
    (dict(self_index=torch.zeros(19, dtype=torch.int64)), ["self_index"]), (dict(self_index=torch.zeros(20)), ["self_index"])])
def test_class_distance_sums_rejections(kwargs, names):
    kw = dict(q=_z(), bank=_z(30), labels=_l(30), num_classes=4)
    kw.update(kwargs)
    _rejected(eae_amd.class_distance_sums, kw, names)


@pytest.mark.parametrize("fn", ["silhouette_samples", "silhouette_score", "class_distance_matrix", "davies_bouldin_score",
                                "calinski_harabasz_score"])
def test_metric_functions_rejections(fn):
    f = getattr(eae_amd, fn)
    base = dict(z=_z(), labels=_l(), num_classes=4)
    bad = [(dict(z=torch.zeros((20, 8), dtype=torch.float64)), ["z "]), (dict(z=torch.zeros((20, 8, 1))), ["z "]),
           (dict(z=torch.zeros((20, 300))), ["width"]), (dict(labels=_l(21)), ["labels"]), (dict(labels=torch.zeros(20)), ["labels"]),
           (dict(labels=torch.zeros(20, dtype=torch.int64, device="meta")), ["labels"]),
           (dict(num_classes=0), ["num_classes"]), (dict(num_classes=257), ["num_classes"]), (dict(num_classes=1.5), ["num_classes"])]
    if fn in ("silhouette_samples", "silhouette_score"):
        bad += [(dict(metric="l1"), ["metric"]), (dict(metric=None), ["metric"])]
    else:
        bad += [(dict(num_classes=None), ["num_classes"])]
    if fn in ("silhouette_score", "class_distance_matrix"):
        bad += [(dict(sample=0), ["sample"]), (dict(sample=21), ["sample"]), (dict(sample=2.0), ["sample"]), (dict(sample=True), ["sample"])]
    for kwargs, names in bad:
        kw = dict(base)
        kw.update(kwargs)
        _rejected(f, kw, names)
    with pytest.raises(RuntimeError, match="HIP device"):                  # all of it passes: only the device is missing
        f(**base)


def test_select_k_rejections():
    bad = [(dict(ks=()), ["ks"]), (dict(ks=5), ["ks"]), (dict(ks=(2, 21)), ["k = 21"]), (dict(ks=(0, 2)), ["k "]), (dict(ks=(2, 257)), ["k "]),
           (dict(ks=(2.0,)), ["k "]), (dict(criterion="gap"), ["criterion"]), (dict(sample=0), ["sample"]), (dict(sample=21), ["sample"]),
           (dict(z=torch.zeros((20, 8), dtype=torch.float64)), ["z "]), (dict(max_iter=-1), ["max_iter"]), (dict(tol=1.5), ["tol"])]
    for kwargs, names in bad:
        kw = dict(z=_z(), ks=(2, 3))
        kw.update(kwargs)
        _rejected(eae_amd.select_k, kw, names)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.select_k(_z(), (2, 3, 20), criterion="davies_bouldin", sample=20)


# ---------------------------------------------------------------------------------------------------- select_k's data separates
def test_six_blobs_win_under_every_criterion_by_more_than_the_bound():
    """What `test_gpu_validity` asks of `select_k` holds in float64 with room to spare: on blobs(2000, 64, 6, 0), clustered by `fit_ref`
    for k in (2, 4, 6, 8, 10), k = 6 has the best score under each criterion, for the silhouette by more than the fp32 kernel can move
    it: with the bound of every sum, a is taken at its upper and b at its lower end for k = 6, the other way round for the others.
    The two indices are float64 on either side (relative error of the order of 1e-12): a fifth is room enough."""
    z, _, _ = blobs(2000, 64, 6, 0)
    rows = np.arange(0, 2000, 4)                                           # a quarter of the rows as queries, against all rows
    lo, hi, db, ch = {}, {}, {}, {}
    for k in (2, 4, 6, 8, 10):
        _, labels, _, counts, _ = fit_ref(z, z[:k])
        assert (counts > 0).all()
        sums, cnt, bound = sums_by_label_ref(z[rows], z, labels, k, rows, 0, center=True)
        s_lo, s_hi = silhouette_range(sums, cnt, bound, labels[rows])
        lo[k], hi[k] = float(s_lo.mean()), float(s_hi.mean())
        db[k], ch[k] = davies_bouldin_ref(z, labels, k), calinski_harabasz_ref(z, labels, k)
    for k in (2, 4, 8, 10):
        assert lo[6] > hi[k] + 0.05, (k, lo, hi)
        assert db[6] < db[k] / 1.2 and ch[6] > 1.2 * ch[k], (k, db, ch)


# ---------------------------------------------------------------------------------------------------- the text table
def test_separation_table():
    nan = float("nan")
    m = np.array([[1.0, 4.0, nan, 2.0], [4.0, 2.0, nan, 8.0], [nan] * 4, [2.0, 8.0, nan, nan]])
    text = eae_amd.separation_table(m, [0.5, -0.25, nan, 0.0], names=["water", "forest", "crop", "road"], digits=2)
    lines = text.splitlines()
    assert lines[0].split() == ["class", "silhouette", "intra", "nearest", "inter", "ratio"] and lines[1] == ""
    assert lines[2].split() == ["water", "0.50", "1.00", "road", "2.00", "2.00"]
    assert lines[3].split() == ["forest", "-0.25", "2.00", "water", "4.00", "2.00"]
    assert lines[4].split() == ["crop", "-", "-", "-", "-", "-"]
    assert lines[5].split() == ["road", "0.00", "-", "water", "2.00", "-"]
    assert eae_amd.separation_table(torch.tensor(m), torch.tensor([0.5, -0.25, nan, 0.0])).splitlines()[2].split()[0] == "0"
    for bad in (dict(matrix=np.zeros((2, 3)), per_class=[0, 0]), dict(matrix=np.zeros((2, 2)), per_class=[0]),
                dict(matrix=np.zeros((2, 2)), per_class=[0, 0], names=["a"])):
        with pytest.raises(ValueError):
            eae_amd.separation_table(**bad)
