"""Nearest-neighbour search without a GPU: the NumPy restatement (tests/knn_ref.py) against plain loops and on hand-worked cases, the
vote rules, the host-only plan of the C library, and every rejection the four functions of `eae_amd.neighbors` make on the host
before a device is needed (all inputs here are CPU tensors: a call that got past its checks fails on the device test)."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from kmeans_ref import blobs
from knn_ref import SHAPES, BOUNDARY_SHAPES, QUERY_TILE, knn_ref, brute_force, vote_ref, accept, bound, distances


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("nq,m,width,k,off", [(5, 7, 3, 3, -1), (4, 2, 2, 3, -1), (6, 6, 2, 2, 0), (3, 9, 1, 4, 2), (1, 1, 1, 1, -1)])
def test_reference_against_plain_loops(nq, m, width, k, off):
    rng = np.random.default_rng(nq * 10 + m)
    q = rng.integers(-3, 4, (nq, width)).astype(np.float32)             # small integers: exact distances, many ties
    bank = rng.integers(-3, 4, (m, width)).astype(np.float32)
    if m > 3:
        bank[2, 0] = np.nan
    if nq > 3:
        q[1, 0] = np.inf
    idx, dist, _ = knn_ref(q, bank, k, off)
    bidx, bdist = brute_force(q, bank, k, off)
    assert np.array_equal(idx, bidx) and np.array_equal(dist, bdist, equal_nan=True)


def test_ties_short_lists_and_self_by_hand():
    bank = np.array([[1.0], [-1.0], [1.0], [3.0], [np.nan]])
    q = np.array([[0.0], [2.0], [np.inf]])
    idx, dist, d = knn_ref(q, bank, 5)
    assert idx.tolist() == [[0, 1, 2, 3, -1], [0, 2, 3, 1, -1], [-1] * 5]
    assert dist[0, :4].tolist() == [1.0, 1.0, 1.0, 9.0] and np.isnan(dist[0, 4]) and np.isnan(dist[2]).all()
    assert np.isinf(d[:, 4]).all() and np.isinf(d[2]).all()
    idx0, _, _ = knn_ref(bank[:4], bank[:4], 2, self_offset=0)
    assert idx0.tolist() == [[2, 1], [0, 2], [0, 1], [0, 2]]
    idx1, _, _ = knn_ref(q[:2], bank, 1, self_offset=1)                  # row 0 may not match 1, row 1 may not match 2
    assert idx1.tolist() == [[0], [0]]


def test_fp32_emulation_meets_the_bound():
    """The acceptance check itself, on an fp32 NumPy emulation of the score: it must pass, with duplicates and a NaN row in the bank."""
    for nq, m, width, k in [s for s in SHAPES if s[0] * s[1] <= 300 * 1031] + [(40, 50, 7, 3)]:
        rng = np.random.default_rng(nq + m + width + k)
        q = rng.standard_normal((nq, width)).astype(np.float32)
        bank = rng.standard_normal((m, width)).astype(np.float32)
        if m > 8:
            bank[5] = bank[1]
            bank[3, 0] = np.nan
        with np.errstate(invalid="ignore"):
            s = (bank * bank).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (q @ bank.T)
            s[:, ~np.isfinite(bank).all(1)] = np.inf
            sp = np.concatenate([s, np.full((nq, max(k - m, 0)), np.inf, dtype=np.float32)], axis=1)
            order = np.argsort(sp, axis=1, kind="stable")[:, :k]
            sc = np.take_along_axis(sp, order, 1)
            dist = np.where(np.isinf(sc), np.nan, np.maximum(sc + (q * q).sum(1, dtype=np.float32)[:, None], 0)).astype(np.float32)
        idx = np.where(np.isinf(sc), -1, order).astype(np.int64)
        accept(q, bank, k, idx, dist)
        assert (bound(q, bank) > 0).all()
    # and it rejects a wrong answer: the farthest row in the first slot
    q, bank = np.zeros((1, 2), dtype=np.float32), np.array([[0, 0], [1, 0], [5, 5]], dtype=np.float32)
    with pytest.raises(AssertionError):
        accept(q, bank, 2, np.array([[2, 0]], dtype=np.int64))
    with pytest.raises(AssertionError):
        accept(q, bank, 2, np.array([[0, 0]], dtype=np.int64))
    accept(q, bank, 2, np.array([[0, 1]], dtype=np.int64))


def test_votes_ties_and_empty_slots():
    labels_of = np.array([2, 0, 2, 1, 7, -1])
    idx = np.array([[0, 1, 3, -1], [1, 3, 0, 2], [4, 5, -1, -1], [-1, -1, -1, -1], [3, 1, 4, 5]])
    dist = np.array([[1.0, 2.0, 4.0, np.nan], [0.5, 0.5, 4.0, 4.0], [1, 1, np.nan, np.nan], [np.nan] * 4, [0.0, 1.0, 2.0, 3.0]])
    lab, votes = vote_ref(idx, dist, labels_of, 3)
    assert votes.tolist() == [[1, 1, 1], [1, 1, 2], [0, 0, 0], [0, 0, 0], [1, 1, 0]]
    assert lab.tolist() == [0, 2, -1, -1, 0]                             # three-way and two-way ties go to the lowest class; no vote: -1
    lab, votes = vote_ref(idx, dist, labels_of, 3, "distance")
    assert lab.tolist() == [2, 0, -1, -1, 1]                             # row 1: classes 0 and 1 tie exactly
    assert votes[0].tolist() == pytest.approx([0.5, 0.25, 1.0]) and votes[1].tolist() == pytest.approx([2.0, 2.0, 0.5])
    assert votes[4, 1] == pytest.approx(1e12) and votes[4, 0] == pytest.approx(1.0)


def test_blob_recipe_is_unanimous():
    """The recipe of the GPU classification test: within-blob d^2 <= 0.01, between-blob d^2 >= 21, tau about 0.001, so every
    neighbour list with k <= 32 of a 600-row, 10-blob set is unanimous under leave-one-out."""
    z, ids, _ = blobs(600, 64, 10, seed=5)
    d = distances(z, z)
    same = ids[:, None] == ids[None, :]
    assert d[same].max() <= 0.01 and d[~same].min() >= 21.0 and bound(z, z).max() < 0.002
    idx, dist, _ = knn_ref(z, z, 32, self_offset=0)
    assert (ids[idx] == ids[:, None]).all() and (idx != np.arange(600)[:, None]).all()
    for w in ("uniform", "distance"):
        assert np.array_equal(vote_ref(idx, dist, ids, 10, w)[0], ids)


# ---------------------------------------------------------------------------------------------------- C ABI, host only
def test_plan_is_host_only_and_deterministic():
    lib = _lib.load()
    slices = {}
    for nq, m, width, k in SHAPES + BOUNDARY_SHAPES + [(1 << 20, 8192, 64, 10), (16, 1 << 20, 64, 10), (2 ** 31 - 1, 2 ** 31 - 1, 256, 32)]:
        s = lib.eae_knn_slices(nq, m, width, k)
        b = lib.eae_knn_workspace_bytes(nq, m, width, k)
        assert s >= 1 and b >= 0 and (b > 0) == (s > 1), (nq, m, width, k, s, b)
        assert b <= 64 << 20 and b % 8 == 0
        assert (s, b) == (lib.eae_knn_slices(nq, m, width, k), lib.eae_knn_workspace_bytes(nq, m, width, k))
        slices[nq, m, width, k] = s
    assert slices[1, 1, 1, 1] == 1 and slices[1000, 4096, 64, 10] > 1 and slices[33, 70001, 64, 10] > 1 and slices[1, 5000, 64, 10] > 1
    assert any(slices[s] == 1 for s in SHAPES) and any(slices[s] > 1 for s in SHAPES)
    assert slices[1 << 20, 8192, 64, 10] == 1 and slices[16, 1 << 20, 64, 10] >= 256       # few queries: the bank split fills the device
    assert slices[BOUNDARY_SHAPES[-1]] == 1 and BOUNDARY_SHAPES[-1][0] > 512 * QUERY_TILE
    for nq, m, width, k in ((0, 5, 4, 1), (-1, 5, 4, 1), (2 ** 31, 5, 4, 1), (5, 0, 4, 1), (5, 2 ** 31, 4, 1), (5, 5, 0, 1), (5, 5, 257, 1),
                            (5, 5, 4, 0), (5, 5, 4, 33)):
        assert lib.eae_knn_slices(nq, m, width, k) < 0 and b"knn" in lib.eae_last_error()
        assert lib.eae_knn_workspace_bytes(nq, m, width, k) < 0


def test_search_rejects_bad_arguments_before_any_launch():
    """EAE_ERR_ARG comes from the host-side checks: no device is touched (this test runs without one)."""
    lib = _lib.load()
    p = 0x1000          # never dereferenced on the host
    ws = 1 << 40
    for nq, m, width, k in ((0, 5, 4, 1), (2 ** 31, 5, 4, 1), (5, 0, 4, 1), (5, 2 ** 31, 4, 1), (5, 5, 0, 1), (5, 5, 257, 1), (5, 5, 4, 0),
                            (5, 5, 4, 33)):
        assert lib.eae_knn_search(None, p, nq, p, m, width, k, -1, p, p, p, ws) == -2
    assert lib.eae_knn_search(None, None, 5, p, 5, 4, 1, -1, p, p, p, ws) == -2
    assert lib.eae_knn_search(None, p, 5, None, 5, 4, 1, -1, p, p, p, ws) == -2
    assert lib.eae_knn_search(None, p, 5, p, 5, 4, 1, -1, None, p, p, ws) == -2
    assert lib.eae_knn_search(None, p, 5, p, 5, 4, 1, -2, p, p, p, ws) == -2 and b"self_offset" in lib.eae_last_error()
    need = lib.eae_knn_workspace_bytes(1, 5000, 64, 10)
    assert need > 0
    assert lib.eae_knn_search(None, p, 1, p, 5000, 64, 10, -1, p, p, None, need) == -2
    assert lib.eae_knn_search(None, p, 1, p, 5000, 64, 10, -1, p, p, p, need - 1) == -2 and b"workspace" in lib.eae_last_error()


# ---------------------------------------------------------------------------------------------------- Python rejections
def _z(n=20, width=8):
    return torch.zeros((n, width), dtype=torch.float32)


def test_exports():
    for name in ("knn_search", "knn_classify", "similar_windows", "knn_classify_scene", "KNNResult"):
        assert name in eae_amd.__all__ and getattr(eae_amd, name) is getattr(eae_amd.neighbors, name)


@pytest.mark.parametrize("kwargs", [
    dict(k=0), dict(k=33), dict(k=2.0), dict(k=True), dict(k=3, metric="l1"), dict(k=3, bank=torch.zeros((5, 7))),
    dict(k=3, bank=torch.zeros((5, 8), dtype=torch.float64)), dict(k=3, bank=torch.zeros(8)), dict(k=3, bank=torch.zeros((0, 8))),
    dict(k=3, queries=torch.zeros((4, 257)), bank=torch.zeros((4, 257))), dict(k=3, queries=np.zeros((4, 8), dtype=np.float32)),
    dict(k=3, exclude_self=True, bank=torch.zeros((21, 8)))])
def test_knn_search_rejections(kwargs):
    kw = dict(queries=_z(), bank=_z(30))
    kw.update(kwargs)
    with pytest.raises(RuntimeError) as e:
        eae_amd.knn_search(**kw)
    assert "HIP device" not in str(e.value)


def test_knn_search_and_classify_need_only_the_device():
    z = _z()
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.knn_search(z, _z(30), 32)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.knn_search(z, z, 3, exclude_self=True, metric="cosine")
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.knn_search(z, _z(20), 3, exclude_self=True)            # equal shapes will do
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.knn_classify(z, _z(30), torch.zeros(30, dtype=torch.int64), 3, 4, weights="distance")


@pytest.mark.parametrize("kwargs", [
    dict(k=0), dict(k=33), dict(num_classes=0), dict(num_classes=2.5), dict(num_classes=True), dict(weights="rank"),
    dict(bank_labels=torch.zeros(29, dtype=torch.int64)), dict(bank_labels=torch.zeros(30)), dict(bank_labels=torch.zeros((30, 1), dtype=torch.int64)),
    dict(bank_labels=[0] * 30), dict(metric="dot"), dict(exclude_self=True)])
def test_knn_classify_rejections(kwargs):
    kw = dict(queries=_z(), bank=_z(30), bank_labels=torch.zeros(30, dtype=torch.int64), k=3, num_classes=4)
    kw.update(kwargs)
    with pytest.raises(RuntimeError) as e:
        eae_amd.knn_classify(**kw)
    assert "HIP device" not in str(e.value)


def _scene_case():
    model = eae_amd.SupervisedAutoencoder(64, 10, image_size=64, in_channels=3)
    return model, torch.zeros((3, 160, 224), dtype=torch.uint8)         # a 2 x 3 grid at the default stride


def test_similar_windows_rejections():
    model, scene = _scene_case()
    ids = torch.tensor([0, 5])
    bad = [dict(query=ids, k=0), dict(query=ids, k=32), dict(query=torch.zeros((2, 64)), k=33), dict(query=torch.tensor([0, 6]), k=2),
           dict(query=torch.tensor([-1]), k=2), dict(query=torch.zeros(0, dtype=torch.int64), k=2), dict(query=torch.zeros((2, 32)), k=2),
           dict(query=torch.zeros((2, 64), dtype=torch.float64), k=2), dict(query=torch.tensor([0, 1], dtype=torch.int32), k=2),
           dict(query=ids, k=2, metric="l1"), dict(query=ids, k=2, windows=torch.tensor([0, 1]), nodata=0), dict(query=ids, k=2, stride=65),
           dict(query=ids, k=2, border="wrap"), dict(query=ids, k=2, rule="some"), dict(query=ids, k=2, max_invalid=1.0),
           dict(query=ids, k=2, nodata=0.5), dict(query=ids, k=2, mask=torch.zeros((5, 5), dtype=torch.bool)),
           dict(query=ids, k=2, windows=torch.tensor([0.5, 1.0])), dict(query=ids, k=2, windows=torch.zeros(0, dtype=torch.int64))]
    for kw in bad:
        with pytest.raises(RuntimeError) as e:
            eae_amd.similar_windows(scene, model, **kw)
        assert "HIP device" not in str(e.value), kw
    with pytest.raises(RuntimeError) as e:
        eae_amd.similar_windows(scene, torch.nn.Linear(2, 2), ids, 2)
    assert "Encoder" in str(e.value)
    for kw in (dict(query=ids, k=31), dict(query=torch.zeros((2, 64)), k=32), dict(query=torch.tensor([0, 11]), k=2, border="reflect")):
        with pytest.raises(RuntimeError, match="HIP device"):
            eae_amd.similar_windows(scene, model, **kw)


def test_knn_classify_scene_rejections():
    model, scene = _scene_case()
    bank, lab = torch.zeros((9, 64)), torch.zeros(9, dtype=torch.int64)
    ok = dict(bank=bank, bank_labels=lab, k=3, num_classes=4)
    bad = [dict(k=0), dict(k=33), dict(bank=torch.zeros((9, 32))), dict(bank=bank.double()), dict(bank=torch.zeros(64)),
           dict(bank_labels=torch.zeros(8, dtype=torch.int64)), dict(bank_labels=lab.float()), dict(num_classes=0), dict(weights="rank"),
           dict(metric="l1"), dict(windows=torch.tensor([0, 1]), nodata=0), dict(stride=65), dict(border="wrap"), dict(rule="some"),
           dict(max_invalid=1.0), dict(nodata=0.5), dict(mask=torch.zeros((5, 5), dtype=torch.bool)),
           dict(windows=torch.zeros(0, dtype=torch.int64))]
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(RuntimeError) as e:
            eae_amd.knn_classify_scene(scene, model, **args)
        assert "HIP device" not in str(e.value), kw
    with pytest.raises(RuntimeError) as e:
        eae_amd.knn_classify_scene(torch.zeros((3, 160, 224), dtype=torch.int32), model, **ok)
    assert "dtype" in str(e.value)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.knn_classify_scene(scene, model, **ok)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.knn_classify_scene(scene, model, weights="distance", metric="cosine", border="edge", **ok)
