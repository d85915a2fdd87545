"""Latent clustering on the device (eae_amd.cluster): `eae_kmeans_assign` / `eae_kmeans_update` through the C ABI by shape against
the NumPy float64 restatement (tests/kmeans_ref.py), then `kmeans_fit`, `kmeans_init` and `cluster_scene`.

Bounds (derived, not measured; kmeans_ref.tau / update_bound): a label is accepted when its float64 distance is within tau_n of the
row's minimum, dist within tau_n of the float64 value, a centroid within (n_k + 1) 2^-24 sum |z| / n_k of the float64 mean.  Counts,
`changed`, ties between equal centroids and everything called "bitwise" are exact."""
import warnings

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from kmeans_ref import assign_ref, update_ref, fit_ref, tau, update_bound, blobs
from scene_util import _model, _scene, _divisor

pytestmark = pytest.mark.gpu

#          (N, L, K)
SHAPES = [(1, 1, 1), (63, 3, 2), (64, 4, 10), (65, 48, 17), (257, 64, 256), (1000, 128, 33),
          (3, 64, 10),                 # N < K
          (1031, 256, 256),
          (70001, 64, 10)]             # 547 row tiles for 512 workgroups: more than one grid round
POISON = -7


def _data(n, width, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, width)).astype(np.float32), rng.standard_normal((k, width)).astype(np.float32)


def _c_assign(z, c, labels=None, have_prev=0, want_dist=True, want_changed=False):
    """One assign call on poisoned outputs: (labels, dist, changed) as NumPy."""
    n, width = z.shape
    zt, ct = torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda()
    lt = torch.full((n,), POISON, dtype=torch.int64, device="cuda") if labels is None else torch.from_numpy(labels).cuda()
    dt = torch.full((n,), float(POISON), dtype=torch.float32, device="cuda") if want_dist else None
    ch = torch.full((1,), POISON, dtype=torch.int64, device="cuda") if want_changed else None
    _lib.check(_lib.load().eae_kmeans_assign(_stream(), _ptr(zt), n, width, _ptr(ct), c.shape[0], _ptr(lt), have_prev, _ptr(dt), _ptr(ch)))
    return lt.cpu().numpy(), None if dt is None else dt.cpu().numpy(), None if ch is None else int(ch.item())


def _c_update(z, labels, c, ws_bytes=None, ws_null=False):
    n, width = z.shape
    k = c.shape[0]
    lib = _lib.load()
    need = lib.eae_kmeans_workspace_bytes(n, width, k)
    assert need > 0
    zt, lt, ct = torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(c).cuda()
    cnt = torch.full((k,), POISON, dtype=torch.int64, device="cuda")
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(nb, 1),), 0xFF, dtype=torch.uint8, device="cuda")          # NaN bit patterns: every partial read must have been written
    rc = lib.eae_kmeans_update(_stream(), _ptr(zt), n, width, _ptr(lt), k, _ptr(ct), _ptr(cnt), None if ws_null else _ptr(ws), nb)
    return rc, ct.cpu().numpy(), cnt.cpu().numpy()


def _bits_equal(a, b):
    """torch.equal on the bit patterns: NaN (the dist of a non-finite row) equals itself."""
    view = {torch.float32: torch.int32, torch.float64: torch.int64}
    return a.dtype == b.dtype and torch.equal(a.view(view.get(a.dtype, a.dtype)), b.view(view.get(b.dtype, b.dtype)))


def _same(res, ref):
    return res.n_iter == ref.n_iter and all(_bits_equal(a, b) for a, b in zip(res[:5], ref[:5]))


def _accept(z, c, labels, dist=None):
    """Every row, none left out: the label's float64 distance within tau_n of the minimum; dist within tau_n of that distance."""
    d64, ref = assign_ref(z, c)
    t = tau(z, c)
    ok = ref >= 0
    assert np.array_equal(labels >= 0, ok) and (labels[~ok] == -1).all()
    assert ((labels[ok] >= 0) & (labels[ok] < c.shape[0])).all()
    got = d64[ok, labels[ok]]
    assert (got - d64[ok].min(axis=1) <= t[ok]).all()
    if dist is not None:
        assert np.isnan(dist[~ok]).all()
        assert (dist[ok] >= 0).all() and (np.abs(dist[ok].astype(np.float64) - got) <= t[ok]).all()
    return d64, ref


# ---------------------------------------------------------------------------------------------------- 1. assign
@pytest.mark.parametrize("n,width,k", SHAPES)
def test_assign_by_shape(n, width, k):
    z, c = _data(n, width, k, seed=n + width + k)
    labels, dist, _ = _c_assign(z, c)
    _accept(z, c, labels, dist)
    # changed against a given previous labelling; dist = NULL leaves only the labels
    prev = np.random.default_rng(n).integers(-1, k, n).astype(np.int64)
    again, none, changed = _c_assign(z, c, labels=prev.copy(), have_prev=1, want_dist=False, want_changed=True)
    assert none is None and np.array_equal(again, labels)
    assert changed == int((prev != labels).sum())


@pytest.mark.parametrize("n,width,k", [(65, 48, 17), (300, 64, 70), (257, 64, 256), (40, 5, 3)])
def test_duplicated_centroids_lower_index_wins(n, width, k):
    z, c = _data(n, width, k, seed=7 * n)
    dup = np.random.default_rng(k).permutation(k)
    c[dup[k // 2:]] = c[dup[:k - k // 2]]                      # every centroid of the second half copies one of the first
    labels, _, _ = _c_assign(z, c)
    _accept(z, c, labels)
    first = np.array([np.flatnonzero((c == c[q]).all(1))[0] for q in range(k)])
    assert np.array_equal(first[labels], labels)               # the label is the lowest index among its equals
    # all centroids equal: every row goes to 0
    c[:] = c[0]
    assert (_c_assign(z, c)[0] == 0).all()


@pytest.mark.parametrize("n,width,k", [(200, 64, 10), (131, 67, 40), (64, 1, 2)])
def test_non_finite_rows(n, width, k):
    z, c = _data(n, width, k, seed=n)
    clean, dclean, _ = _c_assign(z, c)
    bad = {3: (0, np.nan), 17: (width // 2, np.inf), 31: (width - 1, -np.inf), 32: (width - 1, np.nan), n - 1: (0, np.inf)}
    for row, (col, v) in bad.items():
        z[row, col] = v
    labels, dist, _ = _c_assign(z, c)
    rows = np.array(sorted(bad))
    assert (labels[rows] == -1).all() and np.isnan(dist[rows]).all()
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    assert np.array_equal(labels[keep], clean[keep]) and np.array_equal(dist[keep], dclean[keep])      # neighbours undisturbed, bit for bit
    _accept(z, c, labels, dist)


def test_assign_does_not_depend_on_its_neighbours():
    """Rows are independent: a row's label and distance are the same in a long batch and alone (another grid, another tile)."""
    z, c = _data(1500, 48, 33, seed=3)
    labels, dist, _ = _c_assign(z, c)
    for lo, hi in ((0, 1), (700, 701), (129, 400), (1499, 1500)):
        l2, d2, _ = _c_assign(z[lo:hi].copy(), c)
        assert np.array_equal(l2, labels[lo:hi]) and np.array_equal(d2, dist[lo:hi])


# ---------------------------------------------------------------------------------------------------- 2. update
def _labels_for(n, k, seed):
    """Random labels with -1, values >= K and, for K > 1, at least one empty cluster."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(-1, k + 2, n).astype(np.int64)
    if k > 1:
        lab[lab == k // 2] = -1
    if n > 4:
        lab[1], lab[n // 2] = k + 5, -3
    return lab


@pytest.mark.parametrize("n,width,k", SHAPES)
def test_update_by_shape(n, width, k):
    z, c = _data(n, width, k, seed=2 * n + k)
    lab = _labels_for(n, k, seed=n)
    ref, ref_cnt = update_ref(z, lab, c)
    rc, got, cnt = _c_update(z, lab, c)
    assert rc == 0
    assert np.array_equal(cnt, ref_cnt)
    if k > 1:
        assert ref_cnt[k // 2] == 0
    empty = ref_cnt == 0
    assert np.array_equal(got[empty], c[empty])                                    # bitwise unchanged
    bound = update_bound(z, lab, k)
    assert (np.abs(got[~empty].astype(np.float64) - ref[~empty]) <= bound[~empty]).all()
    rc2, got2, cnt2 = _c_update(z, lab, c)
    assert rc2 == 0 and np.array_equal(got2.view(np.uint32), got.view(np.uint32)) and np.array_equal(cnt2, cnt)


def test_update_rejects_a_short_or_missing_workspace():
    z, c = _data(300, 64, 10, seed=1)
    lab = _labels_for(300, 10, seed=2)
    need = _lib.load().eae_kmeans_workspace_bytes(300, 64, 10)
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_null=True)):
        rc, got, cnt = _c_update(z, lab, c, **kw)
        assert rc == -2 and b"workspace" in _lib.load().eae_last_error()
        assert np.array_equal(got, c) and (cnt == POISON).all()                    # nothing was launched


# ---------------------------------------------------------------------------------------------------- 3. fit: exact trajectory
@pytest.mark.parametrize("n,width,k", [(3000, 64, 10), (1000, 3, 4), (5000, 256, 17)])
def test_fit_exact_trajectory(n, width, k):
    z, ids, init = blobs(n, width, k, seed=n + width)
    trace = []
    c_ref, lab_ref, d_ref, cnt_ref, it_ref = fit_ref(z, init, trace=trace)
    for d64, _, cc in trace:                                   # the recipe's margins: no fp32 rounding can move a label
        s = np.sort(d64, axis=1)
        assert ((s[:, 1] - s[:, 0]) > 100 * tau(z, cc)).all()
    zt = torch.from_numpy(z).cuda()
    res = eae_amd.kmeans_fit(zt, k, init=torch.from_numpy(init).cuda())
    assert isinstance(res, eae_amd.KMeansResult) and res.n_iter == it_ref
    labels = res.labels.cpu().numpy()
    assert np.array_equal(labels, lab_ref) and np.array_equal(res.counts.cpu().numpy(), cnt_ref)
    assert (np.abs(res.centroids.cpu().numpy().astype(np.float64) - c_ref) <= update_bound(z, lab_ref, k)).all()
    assert res.inertia.dim() == 0 and res.inertia.dtype == torch.float64 and res.inertia.is_cuda
    assert res.inertia.item() == pytest.approx(res.dist.double().sum().item(), rel=1e-12)
    res2 = eae_amd.kmeans_fit(zt, k, init=torch.from_numpy(init).cuda())
    assert _same(res2, res)


# ---------------------------------------------------------------------------------------------------- 4. fit: properties on random data
@pytest.fixture(scope="module")
def random_fit_data():
    z, c = _data(2000, 16, 8, seed=99)          # (the float64 reference settles after 37 updates from this start)
    z[5, 3], z[77, 0] = np.nan, np.inf
    return z, torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda()


@pytest.mark.parametrize("kwargs", [dict(tol=0.0, max_iter=300), dict(tol=None, max_iter=3)])
def test_fit_result_is_consistent(random_fit_data, kwargs):
    z, zt, init = random_fit_data
    res = eae_amd.kmeans_fit(zt, 8, init=init, **kwargs)
    cent, labels = res.centroids.cpu().numpy(), res.labels.cpu().numpy()
    _accept(z, cent, labels, res.dist.cpu().numpy())                       # labels and dist belong to the returned centroids
    assert labels[5] == -1 and labels[77] == -1
    assert np.array_equal(res.counts.cpu().numpy(), np.bincount(labels[labels >= 0], minlength=8))
    if kwargs["tol"] is None:
        assert res.n_iter == 3
    else:                                                                  # the fixed point: every non-empty centroid is its members' mean
        assert 1 <= res.n_iter < 300
        mean, cnt = update_ref(z, labels, cent)
        ne = cnt > 0
        assert (np.abs(cent[ne].astype(np.float64) - mean[ne]) <= update_bound(z, labels, 8)[ne]).all()


def test_fit_members_mean_after_fixed_updates(random_fit_data):
    """tol=None: the centroids are the means of the labelling of the LAST update, which one assign against the previous centroids gives."""
    z, zt, init = random_fit_data
    prev = eae_amd.kmeans_fit(zt, 8, init=init, tol=None, max_iter=2)
    res = eae_amd.kmeans_fit(zt, 8, init=init, tol=None, max_iter=3)
    members = eae_amd.kmeans_predict(zt, prev.centroids)[0].cpu().numpy()
    assert np.array_equal(members, prev.labels.cpu().numpy())
    mean, cnt = update_ref(z, members, prev.centroids.cpu().numpy())
    ne = cnt > 0
    assert (np.abs(res.centroids.cpu().numpy()[ne].astype(np.float64) - mean[ne]) <= update_bound(z, members, 8)[ne]).all()


def test_inertia_does_not_rise(random_fit_data):
    z, zt, init = random_fit_data
    inertia, slack = [], []
    for j in range(1, 6):
        res = eae_amd.kmeans_fit(zt, 8, init=init, tol=None, max_iter=j)
        inertia.append(res.inertia.item())
        slack.append(np.nansum(tau(z, res.centroids.cpu().numpy())[np.isfinite(z).all(1)]))
    for j in range(4):
        assert inertia[j + 1] <= inertia[j] + slack[j + 1], (j, inertia)


def test_fit_without_tol_reads_nothing_back(random_fit_data):
    z, zt, init = random_fit_data
    ref = eae_amd.kmeans_fit(zt, 8, init=init, tol=None, max_iter=3)      # also the warm-up
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = eae_amd.kmeans_fit(zt, 8, init=init, tol=None, max_iter=3)
        with pytest.raises(RuntimeError):
            got.inertia.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got.n_iter == 3 and _same(got, ref)


# ---------------------------------------------------------------------------------------------------- 5. kmeans_init
def test_kmeans_init():
    k = 7
    z, ids, _ = blobs(2100, 16, k, seed=11)
    bad = [0, 50, 2099]
    z[0, 0], z[50, 7], z[2099, 15] = np.nan, np.inf, -np.inf
    zt = torch.from_numpy(z).cuda()
    c = eae_amd.kmeans_init(zt, k, seed=0).cpu().numpy()
    assert c.shape == (k, 16) and c.dtype == np.float32
    rows = [np.flatnonzero((z.view(np.uint32) == c[q].view(np.uint32)).all(1)) for q in range(k)]
    assert all(len(r) >= 1 for r in rows)                                  # bitwise a row of z
    picked = [int(r[0]) for r in rows]
    assert not set(picked) & set(bad) and np.isfinite(c).all()
    assert sorted(ids[picked].tolist()) == list(range(k))                  # one centroid in every blob
    assert np.array_equal(eae_amd.kmeans_init(zt, k, seed=0).cpu().numpy(), c)
    assert not np.array_equal(eae_amd.kmeans_init(zt, k, seed=1).cpu().numpy(), c)
    # the fit from this seeding recovers the blobs
    res = eae_amd.kmeans_fit(zt, k, seed=0)
    lab = res.labels.cpu().numpy()
    good = lab >= 0
    assert (lab[bad] == -1).all() and good.sum() == 2100 - 3
    assert len(set(zip(lab[good].tolist(), ids[good].tolist()))) == k


def test_kmeans_init_with_fewer_distinct_rows_than_k():
    z = np.repeat(np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32), 5, axis=0)
    z[9] = np.nan
    c = eae_amd.kmeans_init(torch.from_numpy(z).cuda(), 4, seed=3).cpu().numpy()
    assert np.isfinite(c).all() and all((z[:9] == c[q]).all(1).any() for q in range(4))
    assert len({tuple(r) for r in c.tolist()}) == 2
    res = eae_amd.kmeans_fit(torch.from_numpy(z).cuda(), 4, seed=3)
    assert sorted(res.counts.tolist()) == [0, 0, 4, 5]                     # the duplicates keep empty clusters


# ---------------------------------------------------------------------------------------------------- 6. cluster_scene
@pytest.fixture(scope="module")
def scene_case():
    m = _model(3, seed=5, latent=64, batch=16)
    scene = _scene(3, 160, 224, torch.uint8, seed=21)
    return m, scene, _divisor(3, torch.uint8)


def test_cluster_scene_plain_and_windows(scene_case):
    m, scene, div = scene_case
    z = eae_amd.encode_scene(scene, m, divisor=div, stride=32)
    ref = eae_amd.kmeans_fit(z, 4, seed=2)
    cmap, res = eae_amd.cluster_scene(scene, m, k=4, divisor=div, stride=32, seed=2)
    assert cmap.shape == (4, 6) and cmap.dtype == torch.int64 and _same(res, ref)
    assert torch.equal(cmap.reshape(-1), ref.labels) and int(cmap.min()) >= 0
    ids = torch.tensor([20, 3, 7, 11, 12, 0, 23], device="cuda")
    zw = eae_amd.encode_scene(scene, m, divisor=div, stride=32, windows=ids)
    refw = eae_amd.kmeans_fit(zw, 3, seed=1)
    cmapw, resw = eae_amd.cluster_scene(scene, m, k=3, divisor=div, stride=32, windows=ids, seed=1)
    assert _same(resw, refw)
    flat = cmapw.reshape(-1)
    assert torch.equal(flat[ids], refw.labels)
    rest = torch.ones(24, dtype=torch.bool, device="cuda")
    rest[ids] = False
    assert (flat[rest] == -1).all() and (flat[ids] >= 0).all()


def test_cluster_scene_nodata_and_border(scene_case):
    m, scene, div = scene_case
    holed = scene.clone()
    holed[:, :, 100:110] = 0                                               # a stripe of nodata through window columns 2 and 3 (stride 32)
    ids = eae_amd.valid_windows(holed, 64, 32, nodata=0)
    assert 0 < ids.numel() < 24
    ref = eae_amd.kmeans_fit(eae_amd.encode_scene(holed, m, divisor=div, stride=32, windows=ids), 3, seed=4)
    cmap, res = eae_amd.cluster_scene(holed, m, k=3, divisor=div, stride=32, nodata=0, seed=4)
    assert _same(res, ref)
    flat = cmap.reshape(-1)
    rest = torch.ones(24, dtype=torch.bool, device="cuda")
    rest[ids] = False
    assert torch.equal(flat[ids], ref.labels) and (flat[rest] == -1).all() and (flat[ids] >= 0).all()
    with pytest.raises(RuntimeError):
        eae_amd.cluster_scene(holed, m, k=int(ids.numel()) + 1, divisor=div, stride=32, nodata=0)
    # border: the grid that covers the scene
    zb = eae_amd.encode_scene(scene, m, divisor=div, border="reflect")
    refb = eae_amd.kmeans_fit(zb, 5, seed=0)
    cmapb, resb = eae_amd.cluster_scene(scene, m, k=5, divisor=div, border="reflect", seed=0)
    assert cmapb.shape == (3, 4) and _same(resb, refb) and torch.equal(cmapb.reshape(-1), refb.labels)


def test_cluster_scene_with_given_centroids(scene_case):
    m, scene, div = scene_case
    _, fitted = eae_amd.cluster_scene(scene, m, k=4, divisor=div, stride=32, seed=2)
    other = _scene(3, 160, 224, torch.uint8, seed=22)
    cmap, res = eae_amd.cluster_scene(other, m, k=99999, centroids=fitted.centroids, divisor=div, stride=32)
    labels, dist = eae_amd.kmeans_predict(eae_amd.encode_scene(other, m, divisor=div, stride=32), fitted.centroids)
    assert torch.equal(cmap.reshape(-1), labels) and torch.equal(res.labels, labels) and torch.equal(res.dist, dist)
    assert res.n_iter == 0 and torch.equal(res.centroids, fitted.centroids)
    assert torch.equal(res.counts, torch.bincount(labels, minlength=4))
    table = eae_amd.cluster_class_table(cmap, cmap % 2, 4, 2)              # the report helpers take device tensors as they are
    assert table.is_cuda and int(table.sum()) == 24 and eae_amd.name_clusters(table).shape == (4,)
